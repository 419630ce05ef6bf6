// Internal declarations shared by the HIP translation units of librobustcap_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <memory>
#include <string>
#include <type_traits>

// ---- GEMM tiling -------------------------------------------------------------------------------------------
// One workgroup = RC_NW waves = one 32-row x (16*NC)-column output tile; the K range is split across the waves
// (in-workgroup split-K) and reduced through LDS. Each wave runs v_mfma_f32_16x16x4_f32 on 2 row blocks x NC
// column blocks (A: lane l = row l&15, k-quarter l>>4; B: k-quarter l>>4, column l&15).
#define RC_MT 32          // rows per workgroup tile of dense layers (2 MFMA row blocks); LSTM tiles: 16 * mr
#define RC_NT 64          // columns per workgroup tile of dense layers (NC = 4 blocks of 16)
#ifndef RC_NW
#define RC_NW 4           // waves per workgroup (K split)
#endif
#define RC_KC 16          // k per chunk: one dwordx4 (4 consecutive k) per lane per operand block
#define RC_KALIGN 128     // padded K granularity (>= 2 * RC_KC * RC_NW: an even number of chunks per wave)
#define RC_HBUF 3          // copies of every hidden state h: step s writes copy s % 3 and reads copy (s - 1) % 3. Two would do for the
                           // recurrence; the third lets the first wide launch of a wavefront tick (which writes copy (s + 2) % 3)
                           // start while linear2 of the previous tick -- second stream -- still reads copy s % 3
#define RC_MAX_PROB 14    // problems fused in one launch (GemmLaunch travels as a kernel argument: 14 x 232 B = 3.2 KB; no scratch copy: checked in the ISA)

// Every GEMM A operand (sub-net inputs, relu(linear1), hidden states) is stored in MFMA A-fragment order so that a
// wave's A load is one contiguous 1 KiB piece, exactly like the packed weights: for 16-row block row / 16 and
// 16-wide k chunk k / 16 the 256 floats [k-quarter (k/4)&3][row & 15][k & 3] are contiguous. (Row-major rows would
// make each dwordx4 load touch many cache lines; the vector-memory front end, not HBM, was the bound -- profiles/.)
__host__ __device__ inline long long rc_pk(long long row, int k, int ld) {
    return (row >> 4) * (16ll * ld) + (long long)(k >> 4) * 256 + ((k >> 2) & 3) * 64 + (row & 15) * 4 + (k & 3);
}

enum { RC_EPI_DENSE = 0, RC_EPI_RELU = 1, RC_EPI_LSTM = 2 };
enum { RC_PAR_NONE = 0, RC_PAR_SRC = 1, RC_PAR_DST = 2 };

// row flags (one byte per row, rebuilt every frame)
#define RC_ROW_VIS 1u     // rnn4 steps on the camera keypoints   (c > lo or first_frame)
#define RC_ROW_PC 2u      // rnn6 steps on the camera keypoints   (c > lo)
#define RC_ROW_UPD 4u     // vision updater: rnn6/rnn4 step on re-projected landmarks (c <= lo)
#define RC_ROW_REACH 8u   // rnn2 state re-initialised by init_net this frame
#define RC_ROW_MASK 16u   // caller-supplied mask (rc_lstm_step)
// second flag byte (flags2): scheduling of the DEFERRED vision-updater steps. The updater's rnn6/rnn4 steps of
// frame t only change state that frame t+1 reads, so they are executed at the start of frame t+1: merged into that
// frame's own rnn4 / rnn6 launch when the row does not step there anyway (the row just reads its "late" input
// buffer), or in a small transition launch first when it does (regime change low -> high).
#define RC_ROW2_TR 1u     // pending updater step AND the row steps again this frame: transition launch
#define RC_ROW2_M4 2u     // rows of the merged rnn4 launch  (VIS | pending)
#define RC_ROW2_M6 4u     // rows of the merged rnn6 launch  (PC  | pending)
#define RC_ROW2_FLUSH 8u  // rc_get_state: run every pending step now
#define RC_ROW2_VALID 16u // per-row-cursor wavefront engine: the row carries a frame in this ring slot (not a bubble)

struct GemmSeg {
    const float* base;      // activation matrix [rows, ld] in rc_pk order
    long long par_stride;   // elements between the RC_HBUF copies (0 if not multi-buffered)
    int ld;
    int K;                  // padded length of this K segment (multiple of RC_KALIGN; 0 = absent)
    int par_mode;           // RC_PAR_*
    int pad_;
};

struct GemmProblem {
    GemmSeg seg[2];         // A = [seg0 | seg1] along K
    const float* W;         // packed weights, see pack_weights() in rc_api.cpp
    const void* Ws;         // the same weights as three bf16 planes (split-bf16 products), see pack_weights_split()
    const float* bias;      // [n_tiles * 64] in packed column order
    float* out;             // dense: out[row * ldo + col0 + n], or rc_pk(row, col0 + n, ldo) if out_packed
    float* hstate;          // lstm: h[parity][row][H]
    float* cstate;          // lstm: c[row][H]
    int* steps;             // per-row step counter of this net (copy = steps % RC_HBUF)
    const unsigned char* flags;
    const float* alt_base;  // seg[0] of rows WITHOUT sel_bit in sel_flags reads here (deferred updater input)
    const unsigned char* sel_flags;
    const unsigned char* out_flags;   // dense: only rows with out_bit set are written (0 = all active rows)
    long long h_par_stride;
    int ldo, N, H;
    int out_col0, out_packed;
    int sel_bit, out_bit;
    int flag_bit;           // 0 = all rows
    int epi;                // RC_EPI_*
    int open_step;          // linear1 opens a step: the n_tile 0 workgroup increments steps[row]
    int n_tiles, m_tiles, wg_base, Kp;
    int nc;                 // 16-column blocks per tile
    int mr;                 // 16-row blocks per tile (2 or 4); (mr, nc) must be one of the instantiated shapes
    int trace_base;         // first record slot of this launch (read by -DRC_TRACE_TILES builds only)
    int nt;                 // live frames: stream THIS problem's weights with non-temporal loads (rc_gemm_small_nt_kernel)
    int step_off;           // added to steps[row] wherever the step parity is formed. Frame-stepped launches: 0 (linear1
                            // has already incremented the counter). Sequence mode: 1 + (frame - first frame of the
                            // segment), with open_step = 0: the counters stand still while stages of several frames are in
                            // flight and are advanced once, after the segment.
};

struct GemmLaunch {
    int n;                  // problems
    int B;                  // rows in the batch
    int split;              // the gemm mode. 1: products as split-bf16 partial products on the bf16 MFMA (rc_gemm.hip: mma_kblock), W -> Ws;
                            // 2: three products of two round-to-nearest planes, every p.Ws then a mode-2 packing (rc_launch_planes2)
    int live;               // 1: launch of a live frame (16-row launches then stream their weights with non-temporal loads)
    GemmProblem p[RC_MAX_PROB];
};

#define RC_TICK_PROB 24   // GEMM problems of one sequence-mode tick (6 sub-nets x {linear1, LSTM l0, LSTM l1, linear2})

// ---- shared-weight gate GEMM of the LSTM layer steps (rc_gemm_lds.hip): 256-row x 128-column tiles, 8 waves, the weight planes of
// a k-block staged once per workgroup in LDS, K halved across two workgroups (seg[0] | seg[1]) that meet through a slab in device memory
#define RC_LDS_MAXP 12    // layer steps fused in one launch
#define RC_LDS_SLAB_FLOATS 65536   // per tile: two half sums of 256 x 128 floats
struct LdsProblem {
    GemmSeg seg[2];         // A = [seg0 | seg1] along K, each H long: the layer's input and its own h(t - 1)
    const void* Ws;         // weight planes (pack_weights_split)
    const float* bias;
    float* hstate;
    float* cstate;
    const int* steps;
    const unsigned char* flags;
    float* slab;            // [tiles][2][256 x 128]: the half sums
    int* tickets;           // [tiles], zero between launches
    long long h_par_stride;
    int H, flag_bit, n_tiles, m_tiles, wg_base, Qs, step_off, ksplit;
    // relu(linear1) as an item of the resident kernel (epi = RC_EPI_RELU; ksplit 1, seg[0] | seg[1] = the two halves of ONE input): out
    // [rows, ldo] in rc_pk order; rows without sel_bit in sel_flags read alt[0] | alt[1] instead (a rider's deferred input)
    float* out;
    const float* alt[2];
    const unsigned char* sel_flags;
    int epi, ldo, sel_bit;
    int block_pick;         // 1: a tile whose active rows fill as many 16-row blocks as it has storage blocks with an active row takes those blocks whole (rc_gemm_lds.hip: block mode)
};
struct LdsLaunch {
    int n, B;
    LdsProblem p[RC_LDS_MAXP];
};
#define RC_RES_MAXP 20    // problems of a tick of the resident kernel: twelve layer steps + six linear1
void rc_launch_gemm_lds(const LdsLaunch& L, int total_wg, hipStream_t s, hipEvent_t stop = nullptr, int planes = 3);   // planes 2: mode 2 (every p.Ws a two-plane packing)
// mode 2's two round-to-nearest bf16 planes [cb][kb][2][lane][8] of a matrix, from its fp32 packing W (rc_gemm.hip: rc_planes2_kernel)
void rc_launch_planes2(const float* W, void* Ws2, int Np, int Kp, hipStream_t s);

// ---- resident layer-step kernel (rc_gemm_lds.hip: rc_gemm_resident_kernel) ----------------------------------
// One launch carries the LSTM layer steps of EVERY tick of a wavefront-engine segment: its workgroups stay on their CUs and take work
// items (the items of rc_gemm_lds_kernel, tick after tick, longest first inside a tick) from one queue in device memory. What stream
// order and events did between launches, counters in device memory do between items (rc_sequence_api.cpp: run_resident_segment).
struct ResidentTick {
    int n, B;                             // the tick's problems, as one launch of the shared-weight kernel would carry them
    LdsProblem p[RC_RES_MAXP];
    int n_items;                          // work items of the tick (every problem's range padded to a multiple of 8)
    int dep[RC_RES_MAXP][2];              // per problem: up to two problems of the PREVIOUS tick it reads (own h(t - 1); its input: layer 0's h, relu(linear1)), -1 = none
    int dep_items[RC_RES_MAXP][2];        // ... and their item counts
    int need_tail[RC_RES_MAXP];           // 1: the problem reads what the previous tick's second-stream chain wrote (linear1: fuse / tail / prep; rnn2 behind an init_net state write)
};
struct ResidentArgs {
    const ResidentTick* ticks;
    const int* item_base;                 // [n_ticks + 1] first queue position of every tick
    int n_ticks;
    int* head;                            // queue head
    int* done;                            // [n_ticks][RC_RES_MAXP] items finished per (tick, problem)
    int* tick_done;                       // [n_ticks] items finished per tick
    const int* flag_tail;                 // second stream: tails finished (the chain of tick k done -> k + 1)
    int* abort;                           // set by whoever waited longer than the bound; everybody else stops waiting
    unsigned long long spin_bound;        // wall_clock64 ticks (100 MHz)
};
void rc_launch_gemm_resident(const ResidentArgs& R, int workgroups, hipStream_t s);
void rc_launch_flag_set(int* flag, int value, hipStream_t s);
void rc_launch_flag_wait(const int* counter, int target, int* abort, unsigned long long spin_bound, hipStream_t s);

// ---- per-frame small kernels -------------------------------------------------------------------------------
struct BodyConst {          // device copy of the body constants the path needs
    int parent[24];
    int level[24];          // depth in the kinematic tree
    float bone[24][3];      // rest bone vectors  (j_rest[i] - j_rest[parent[i]])
    float jrest[24][3];     // rest joints, root at the origin
    float jroot[3];         // rest position of the root joint (subtracted from the template, model.py:87)
    float w33[33][24];
    float v33[33][3];       // landmark vertices, root-relative
    int override_joint[33]; // sync_mp3d: landmark row -> joint id, or -1
    int nchild[24];         // children of a joint, ascending (the reverse sweep of the smplify gradient pulls from them)
    int child[24][4];
};

struct FrameBuffers {       // device pointers owned by the context (all [B, ld] row-major)
    float *x2, *x3, *x4, *x6, *x78, *x4l, *x6l, *xi;   // concatenated sub-net inputs (rc_pk order, padded, pads stay zero)
    float *vr, *pc, *r6d, *contact;                     // sub-net outputs consumed by the fusion logic
    float *init_out;                                    // rnn2.init_net output [B, 2048]
    unsigned char* flags;                               // RC_ROW_* per row
    unsigned char* flags2;                              // RC_ROW2_* per row
    unsigned char* pend;                                // 1 = updater step of the previous frame still to run
    unsigned char* regime;                              // 0 low / 1 mid / 2 high
    double* kconf;                                      // (c - lo) / (hi - lo) per row
    float* gravity;                                     // [B,3]
    // per-row fusion state (net/sig_mp.py:85-90)
    float *last_pfoot, *last_tran, *floor, *j_temp;
    int *has_last, *n_floor, *first_reach, *uv_count;
    int* trace;                                         // [B,8]
    // rnn2 state for the init_net write
    float *h2, *c2;
    int* steps2;
    long long h2_par_stride, h2_layer_stride, c2_layer_stride;
    // per-row-cursor wavefront engine (ring slots only; nullptr in the context's own frame-stepped buffers):
    int* frame;             // [B] frame index (relative to the call) the row carries in this slot, -1 = bubble
    int* wsteps;            // [6][B] step number of each sub-net for the step this slot's frame (or rider) takes
};

// rc_prep_wave_kernel: which frame every row starts at this tick (host plan), the global step counters it opens steps on,
// and the context's own updater-input buffers (a deferred updater step pending from before the segment rides the first slot)
struct WavePrep {
    const int* frame_at;    // [B] of this tick
    int* steps[6];          // the sub-nets' per-row step counters
    const float *cx4l, *cx6l;
    int first_tick;
    int t0;                 // first frame of the segment: a row whose frames end in front of it keeps its pending step
};
// rc_tail_kernel in the per-row-cursor engine: the vision updater's two sub-net steps of a frame "ride" the ring slot that
// is initialised at the tick its tail runs (target slot); the last frame of the segment leaves them pending instead.
struct WaveTail {
    int on;                 // 0 = frame-stepped / all-visible engine
    int t_last;             // last frame of the segment
    float *x4l, *x6l;       // target slot
    unsigned char* flags2;
    int* wsteps;
    int *steps4, *steps6;   // global step counters of rnn4 / rnn6
    float *cx4l, *cx6l;     // the context's own buffers (pending step of the last frame)
};

struct FrameIO {
    const float *j2d, *acc, *ori, *first_tran;
    float *pose_out, *tran_out;
    long long s_j2d, s_acc, s_ori, s_pose, s_tran;      // row strides (elements)
    // rc_sequence_rows: row b of the call runs frames 0 .. len[b] - 1 only (DEVICE int32[B]; nullptr = every row runs every frame).
    // t = index, in the call `len` belongs to, of the frame these pointers stand at (a ring slot's frame index counts from it).
    const int* len;
    int t;
};
// "row `row` has a frame at call index `t`" / "... and it is the row's last of the call" (wave-uniform where a wave owns a row)
__host__ __device__ inline bool rc_row_live(const FrameIO& io, int row, int t) { return !io.len || t < io.len[row]; }

struct rc_params_dev {
    double conf_lo, conf_hi, tran_filter_num;
    float contact_threshold, distance_threshold, height_threshold;
    int use_flat_floor, use_vision_updater, use_imu_updater, live, update_vision_freq, use_reproj_opt;
    float smooth;
};

// ---- the lean live frame (rc_live.hip; live_server.py:40-48 calls forward_online once per camera frame) -------------------------------
// Batch <= RC_LIVE_MAXB, steady-state frames only (no first frame, no transition step, init_net already run): SEVEN dependent
// launches instead of 11-14 --
//   K1 prep + linear1{rnn4, rnn2} | K2 LSTM l0 | K3 LSTM l1 + per-tile partial sums of linear2 |
//   K4 (sum of the partials, fuse) + linear1{rnn6, rnn3, rnn7, rnn8} | K5 LSTM l0 | K6 LSTM l1 + linear2 partials |
//   K7 (sum of the partials) + tail
// linear2 y = W2 h + b is computed where h is produced: the workgroup that owns 4 (or 8) hidden units multiplies them with its
// columns of W2 and stores the partial y; the consuming kernel sums the partials of all tiles in a FIXED order behind the launch
// boundary (no atomics, no fences, nothing placement-dependent). Every kernel requests its weights first and its per-row words
// (flags, step parities, cell state) in the same batch: one memory latency in front of the first MFMA instead of a chain of four.
#define RC_LIVE_MAXB 4
// Second argument of the LSTM launches of the lean frame. `hot`: the per-row words a launch needs before its first activation load --
// step number (-> which copy of h) and whether the row steps, per problem of the launch (stage 1: rnn4, rnn2; stage 2: rnn6, rnn3,
// rnn7, rnn8) -- are IN the kernel arguments: on the AQL path (rc_aql.cpp) the arguments live in device memory of the context's own,
// and the linear1 kernel that opens the steps (K1 / K4) writes them there, so the LSTM kernels have no dependent global read in
// front of the weight stream. hot = 0 (graph replay, direct launches): read from the state.
// `pre` (round 5, the idle-time pre-step): 1 = the recurrent half of this launch's layer steps -- the partial sums of waves 2 and 3 of every
// tile, W_hh . h(t - 1) over their K ranges -- was computed after the PREVIOUS frame (rc_live_pre) and sits in `prebuf`; those waves load
// it instead of streaming their half of the weights. Same MFMA chain per accumulator, same reduction order: bitwise the unhoisted step.
struct LiveGrid { int hot; int st[4][RC_LIVE_MAXB]; int act[4][RC_LIVE_MAXB]; int pre; int pre_base; const float* prebuf; };
struct LiveNet {
    const float *W1, *b1;           // linear1: pack_weights order [N/16][Kp1/16][64][4], bias
    const float *Wl[2], *bl[2];     // LSTM layers: pack_weights order, gate-interleaved columns; b_ih + b_hh
    const float *W2, *b2;           // linear2 ROW-MAJOR [out][H] (a unit's column slice is one 16-byte piece per output), bias [out]
    float *x1, *h, *c, *part;       // relu(linear1) [Bp][H] rc_pk | h [2][RC_HBUF][Bp][H] rc_pk | c [2][B][H] | partials [H/UT][RC_LIVE_MAXB][outp]
    int* steps;
    int H, out, outp, Kp1;
    long long BpH;                  // elements between the copies of h
};
struct LiveFrame {
    LiveNet net[6];                 // kNets order: rnn2, rnn3, rnn4, rnn6, rnn7, rnn8
    FrameBuffers fb;
    FrameIO io;
    rc_params_dev prm;
    const BodyConst* body;
    int* status;                    // pinned host word, set != 0 by K1 when the frame is not the lean plan's (a transition step or an init_net trigger:
                                    // the host's mirror of those flags is conservative, this is the check behind it); rc_live_step then replays the full capture
    int* abort;                     // device word K1 writes every frame (0 / 1): set, the frame's kernels change NOTHING (no state, no step counters, no outputs)
    unsigned* spin_mb;              // waiting K1 (rc_live.hip, RC_LIVE_SPIN): its mailbox (one of two, frames alternate) in host-writable device memory -- [0] the host's command (0 none, 1 go,
                                    // 2 skip), [16] the decision workgroup 0 publishes (1 go, 2 skip, 3 timed out); else null
    unsigned* spin_state;           // pinned host word: 3 when the spinning K1 gave up waiting
    LiveGrid* hot[4];               // AQL path: the LiveGrid argument blocks of K2, K3 (written by K1) and K5, K6 (by K4); else null
    unsigned* done_flag;            // AQL path, one row: pinned host word K7 stores the frame's sequence number to, behind a system-scope
    unsigned* done_seq;             // release, when everything of the frame is written (device counter of frames); else null
    int B;
    int nc;                         // 16-column blocks per LSTM tile (1 or 2)
};
#define RC_LIVE_KERNELS 7
struct LiveKernel {             // one launch of the lean frame: host function + symbol name, grid (workgroups of `wg` threads), arguments
    const void* fn;
    const char* name;
    unsigned grid;
    int has_grid;               // arguments: (LiveFrame) or (LiveFrame, LiveGrid)
    unsigned wg;                // threads per workgroup (0 = 256)
    LiveFrame F;
    LiveGrid G;
};
int rc_live_plan(const LiveFrame& F, LiveKernel* out, const float* prebuf = nullptr);   // fills RC_LIVE_KERNELS entries, returns their number;
                                                                      // prebuf: the LSTM launches take their recurrent halves from it (LiveGrid.pre)
int rc_live_pre_plan(const LiveFrame& F, float* prebuf, LiveKernel* out);   // the idle-time pre-step: rc_live_pre (+ rc_live_warm); returns 1 or 2 launches, or 0
long long rc_live_pre_floats(const LiveFrame& F);                     // size of prebuf
void rc_launch_live_frame(const LiveFrame& F, hipStream_t s, const float* prebuf = nullptr);
void rc_launch_live_pre(const LiveFrame& F, float* prebuf, hipStream_t s);

// The same chains as AQL packets on an HSA queue of the context's own (rc_aql.cpp): rc_live_step then pays ~0.5 us of host time to
// enqueue the frame instead of hipGraphLaunch's ~7 us, and polls the completion itself. A chain holds several PROGRAMS (packet lists
// with their own argument blocks) on one queue: the lean frame, the lean frame on pre-computed recurrent halves, and the pre-step.
struct AqlChain;
int rc_aql_create(int hip_device, AqlChain** out, char* err, int err_len);
// a program of n <= RC_LIVE_KERNELS launches; frame != 0: a live frame (its last kernel stores the completion word, its last packet carries
// the frame signal), else a background program (pre-step) with a signal of its own. Returns the program id (>= 0) or -1.
int rc_aql_add(AqlChain* c, const LiveKernel* k, int n, int frame, char* err, int err_len);
int rc_aql_run(AqlChain* c, int prog);                                // frame program: submit, then spin until it retired; 0 = done
int rc_aql_submit(AqlChain* c, int prog);                             // background program: submit and return
int rc_aql_alloc_shared(AqlChain* c, size_t bytes, void** ptr);         // device memory the host can write (large BAR), freed with the chain; 0 = ok
int rc_aql_submit_ahead(AqlChain* c, int prog, int beside);             // a whole frame program submitted without waiting (queued ahead: its K1 waits on the mailbox;
                                                                        // beside: that K1 may start beside the frame in front of it)
unsigned long long rc_aql_seq(const AqlChain* c);                       // number of the frame submitted last
int rc_aql_wait_seq(AqlChain* c, unsigned long long seq);               // spin until frame `seq` has retired
int rc_aql_wait_frame(AqlChain* c);                                     // ... the frame submitted last
int rc_aql_fence_background(AqlChain* c);                               // a barrier packet that counts as a background program (rc_aql_wait_background)
void rc_aql_set_mailbox(AqlChain* c, volatile unsigned* mb);            // the drain tells a K1 still spinning to leave
int rc_aql_arm(AqlChain* c);                         // RC_LIVE_ARM: a barrier-AND packet the next push releases
int rc_aql_wait_background(AqlChain* c);                              // until every submitted background program has retired
void rc_aql_destroy(AqlChain* c);

void rc_launch_gemm(const GemmLaunch& L, int total_wg, hipStream_t s, hipEvent_t stop = nullptr);
void rc_launch_scan_conf(const float* j2d, long long row_stride, int B, int T, double conf_lo, double conf_hi, signed char* codes, hipStream_t s,
                         float* means = nullptr, const int* len = nullptr, int len_t0 = 0);   // len: frames t with len_t0 + t >= len[row] are not read, code -1
void rc_launch_advance_steps(int* const* steps6, int n_frames, int B, hipStream_t s);
bool rc_gemm_is_w32(const GemmLaunch& L);       // true: the launch runs on rc_gemm_split48_w32_kernel
bool rc_gemm_is_small(const GemmLaunch& L);     // true: the launch runs on rc_gemm_small_kernel (16-row tiles only)
void rc_launch_prep(const FrameBuffers& fb, const FrameIO& io, const rc_params_dev& prm, int B, int first_frame, hipStream_t s);
void rc_launch_fuse(const FrameBuffers& fb, const FrameIO& io, const rc_params_dev& prm, int B, hipStream_t s);
void rc_launch_tail(const FrameBuffers& fb, const FrameIO& io, const rc_params_dev& prm, const BodyConst* body, int B,
                    int first_frame, hipStream_t s, const FrameIO* io_next = nullptr,    // io_next: also the next frame's prep
                    const WaveTail* wt = nullptr, hipEvent_t stop = nullptr);   // stop: event signalled by this dispatch
bool rc_launch_fuse_tail(const FrameBuffers& fb_tail, const FrameBuffers& fb_fuse, const FrameIO& io, const rc_params_dev& prm, const BodyConst* body, int B,
                         const WaveTail& wt, hipStream_t s, hipEvent_t stop);   // fuse + tail of a tick in one launch (false: not available, launch them apart)
void rc_launch_prep_wave(const FrameBuffers& slot, const FrameIO& io0, const rc_params_dev& prm, int B, const WavePrep& w, hipStream_t s);
void rc_launch_reset(const FrameBuffers& fb, float* const* h, float* const* c, const int* hidden, const unsigned char* mask,
                     int B, hipStream_t s);

void rc_launch_flush_flags(const FrameBuffers& fb, int B, hipStream_t s);

// ---- row state (rc_rowstate.hip; rc_save_rows / rc_load_rows / rc_set_state in rc_rowstate_api.cpp) ------------------------------------
// One record = everything a row carries from frame to frame, as 32-bit words:
//   per sub-net (kNets order) and layer: h[H] (the copy the row's step counter designates), then c[H]   -- 17,408 words
//   x4l[256], x6l[256]: the row's part of the context's own updater-input buffers (inputs of a pending step)
//   the last RC_ROWSTATE_SMALL words: j_temp[99] floor[33] last_pfoot[6] last_tran[3] gravity[3] | has_last n_floor first_reach uv_count
//   pend | trace[8] | three zero words (the record is a multiple of 16 bytes)
#define RC_ROWSTATE_SMALL 160
#define RC_ROWSTATE_SEGS 27   // 12 h + 12 c + x4l + x6l + the small block: grid.y of the two kernels
enum { RC_RS_PK = 0, RC_RS_ROWS = 1, RC_RS_SMALL = 2 };
struct RowSeg {
    float* base;            // RC_RS_PK: [copies][Bp, ld] in rc_pk order; RC_RS_ROWS: [B, ld] row-major; RC_RS_SMALL: unused (the fields come from fb)
    const int* steps;       // RC_RS_PK: per-row step counter that picks the copy, or nullptr (one copy)
    long long copy_stride;  // elements between the copies
    int ld;                 // words of the segment per row (a multiple of 4)
    int rec_off;            // first word of the segment in a record (a multiple of 4)
    int kind, pad_;
};
struct RowStateArgs { RowSeg seg[RC_ROWSTATE_SEGS]; FrameBuffers fb; long long rec_words; };
// the listed rows of ONE 16-row block of the context (ascending) and the record each of them owns: built and checked on the host, the only
// indices the kernels use
struct RowGroup { int m; int row[16]; int rec[16]; };
// load == false: context -> blob (gather), true: blob -> context (scatter); groups DEVICE [n_groups], blob DEVICE, 16-byte aligned
void rc_launch_rowstate(const RowStateArgs& a, const RowGroup* groups, int n_groups, float* blob, bool load, hipStream_t s);
// rc_set_state: hs / cs DEVICE [2, B, H] row-major or nullptr, mask DEVICE uint8[B] or nullptr; h [2][RC_HBUF][Bp, H] rc_pk, c [2][B, H]
void rc_launch_set_state(const float* hs, const float* cs, const unsigned char* mask, const int* steps, float* h, float* c, int B,
                         long long BpH, int H, hipStream_t s);
void rc_launch_pack_rows(const float* src, int src_ld, int cols, float* dst, int ld, int B, hipStream_t s);

void rc_launch_r6d(const float* r6d, float* R, long long n, hipStream_t s);
struct CamConst { float Kinv[9]; float R[9]; };
void rc_launch_camera_inputs(const float* kp, const float* acc, const float* ori, const CamConst& cam, float* j2dc, float* accc,
                             float* oric, long long n, hipStream_t s);
void rc_launch_shape_body(const float* vt, const float* sd, const float* beta, const float* Jr, int V, float* v, float* j, hipStream_t s);
void rc_launch_fk_r(const BodyConst* body, const float* Rl, float* Rg, long long n, hipStream_t s);
void rc_launch_bone_to_joint(const BodyConst* body, const float* bone, float* joint, long long n, hipStream_t s);
void rc_launch_joint_to_bone(const BodyConst* body, const float* joint, float* bone, long long n, hipStream_t s);
void rc_launch_zero_pose(const BodyConst* body, const float* vt, int V, float* joint, float* vert, hipStream_t s);
void rc_launch_rotmat_to_r6d(const float* R, float* r6d, long long n, hipStream_t s);
void rc_launch_lerp(const float* a, const float* b, float w1, float w2, float* out, long long n, hipStream_t s);
void rc_launch_normalize_rows(const float* x, float* out, float* norm, long long rows, int width, hipStream_t s);
void rc_launch_angle_between(const float* R1, const float* R2, float* out, long long n, hipStream_t s);
void rc_launch_bbox_normalise(const float* kp, float* out, long long n, hipStream_t s);
void rc_launch_camera_inputs_rows(const float* kp, const float* acc, const float* ori, const int* seq_of_row, const int* len,
                                  const CamConst* cams, float sx, float sy, int n_rows, int Tmax, float* j2dc, float* accc,
                                  float* oric, hipStream_t s);
void rc_launch_aa2R(const float* aa, float* R, long long n, hipStream_t s);
void rc_launch_R2aa(const float* R, float* aa, long long n, hipStream_t s);
void rc_launch_ik(const BodyConst* body, const float* Rg, float* Rl, long long n, hipStream_t s);
void rc_launch_fk_bone(const BodyConst* body, const float* Rg, float* joints, long long n, hipStream_t s);
void rc_launch_body_fk(const BodyConst* body, const float* pose, const float* tran, float* grot, float* joint,
                       float* j33, long long n, hipStream_t s);
void rc_launch_body_mesh(const BodyConst* body, const float* vt, const float* w, int V, const float* pose, const float* tran,
                         float* vert, long long n, float* scratch, hipStream_t s);   // scratch: rc_body_mesh_scratch_floats(n)
long long rc_body_mesh_scratch_floats(long long n);
void rc_launch_residual(const BodyConst* body, const float* pose, const float* tran, const float* kp, const float* K,
                        float sigma, unsigned long long ign_mask, float* loss, long long T, hipStream_t s);
#define RC_IGN_DEFAULT 0x1800003FEull     // MediaPipe landmarks {1..9, 31, 32} (temporal_smplify.py:92); use_head: {31, 32}
// kM: regressor folded with the skinning data, [nk][24][4] (rc_api.cpp: fold_regressor), or nullptr (the SMPL joints stand in)
void rc_launch_mesh_metrics(const BodyConst* body, const float* vt, const float* w, int V, const float* kM, int nk, const float* pose_p,
                            const float* pose_t, float* out, long long n, float* scratch, hipStream_t s);
long long rc_mesh_metrics_scratch_floats(int V, long long n);
void rc_launch_imu_frames(const BodyConst* body, const float* vt, const float* w, const int* vid, const int* jid, const float* pose,
                          const float* tran, float* ori, float* joint, float* vert6, long long T, hipStream_t s);
void rc_launch_syn_acc(const float* v, float* acc, long long T, long long width, int n, hipStream_t s);
// ---- motions of a ragged batch of sequences prepared in one pass (rc_prepare.hip; rc_set_shape_space, rc_prepare_motions in rc_prepare_api.cpp)
// One sequence: input frames in0, in0 + step, ... give output frames [out0, out0 + out_n)
struct PrepSeq { long long in0, out0; int step, out_n; };
// The rest body of one sequence, root at the origin: what the joint chain and the 39 skins read (33 landmarks, then 6 IMU vertices)
struct PrepRest { float bone[24][3]; float jrest[24][3]; float v39[39][3]; };
// Device arrays of rc_set_shape_space: Jt [24,3], JS [24,3,10] (nullptr without a shape basis), vt39 [39,3], S39 [39,3,10] (same), w39 [39,24];
// vid: the 39 vertex ids
struct PrepShapeSpace { const float *Jt, *JS, *vt39, *S39, *w39; int vid[39]; };
// tab DEVICE [n_seq]; rest DEVICE [betas ? n_seq : 1]; vert6 DEVICE [frames,6,3] (a scratch where the caller wants none); world_rot, jid HOST
void rc_launch_prepare_motions(const BodyConst* body, const float* mesh_vt, const PrepShapeSpace& sp, const PrepSeq* tab, int n_seq,
                               long long frames, const float* pose_aa, int pose_joints, const float* tran, const float* betas,
                               const float* world_rot, const int* jid, int smooth_n, PrepRest* rest, float* pose_out, float* tran_out,
                               float* ori, float* acc, float* joint, float* sync, float* vert6, float* rest_joint_out, hipStream_t s);
// rc_prepare_camera_motions: per sequence its first camera row and its detector frames [kp0, kp0 + kp_n) (beside a PrepSeq with step 1);
// a camera row is the first three rows of a T_cw
struct PrepCam { long long cam0, kp0; int kp_n, pad; };
struct PrepCamRow { float m[12]; };
// tab, cam DEVICE [n_seq]; cam_rows DEVICE; cam_repeat 0: one row per sequence; sync, kp_in / kp_out may be nullptr; the rest as above
void rc_launch_prepare_camera_motions(const BodyConst* body, const float* mesh_vt, const PrepShapeSpace& sp, const PrepSeq* tab,
                                      const PrepCam* cam, int n_seq, long long frames, int cam_repeat, bool root_only, const float* pose_aa,
                                      const float* tran, const float* betas, const PrepCamRow* cam_rows, const float* kp_in, const int* jid,
                                      int smooth_n, PrepRest* rest, float* pose_out, float* tran_out, float* ori, float* acc, float* joint,
                                      float* sync, float* vert6, float* kp_out, float* rest_joint_out, hipStream_t s);
void rc_launch_procrustes(const float* S1, const float* S2, int nk, float* err, long long n, hipStream_t s);
void rc_launch_point_distance(const float* a, const float* b, float* d, long long n, hipStream_t s);
// ---- FullMotionEvaluator per group of a concatenated batch (rc_motion.hip; rc_motion_metrics in rc_api.cpp) -----------------------------
#define RC_MOTION_FG 32                // frames per workgroup of the column and vertex sweeps; a block holds frames of ONE group
// One group: frames [frame0, frame0 + frames) of the call; its frame blocks are [blk0, blk0 + nblk) of the launch, nblk = ceil(frames / FG)
struct MotionGroup { long long frame0, frames; int blk0, nblk; };
long long rc_motion_scratch_floats(long long n);                                          // per-frame columns, joints and difference transforms
long long rc_motion_partial_doubles(int V, long long blocks, int groups, bool mesh);      // per-block (mean, M2) pairs and the slab sums
// out [groups,11,2], per_joint [groups,4,24] or nullptr; tab DEVICE [groups]; blocks = sum of nblk; mesh == false: no vertex sweep, row 1 NaN
void rc_launch_motion_metrics(const BodyConst* body, const float* vt, const float* w, int V, const MotionGroup* tab, int groups,
                              long long blocks, const float* pose_p, const float* tran_p, const float* pose_t, const float* tran_t, long long n,
                              int fps, int align, unsigned mask, bool mesh, float* scratch, double* partial, float* out, float* per_joint,
                              hipStream_t s);
// ---- the evaluators' SVD alignments (rc_align.hip; rc_svd_rotate and rc_aligned_metrics in rc_api.cpp) --------------------------------
// One listed pair j <= k of the mesh fold: c = C[j,k] = sum_v w[v,j] w[v,k] x~_v x~_v^T, 4x4 row-major (symmetric; C[k,j] is the same matrix)
struct AlignPair { int j, k; double c[16]; };
void rc_launch_svd_rotate(const float* src, const float* dst, long long n, int m, unsigned what, float* R, float* t, float* s, float* moved,
                          hipStream_t st);
long long rc_align_scratch_floats(long long n);                                           // per-frame joint errors and aligned difference transforms
long long rc_align_partial_doubles(int V, long long n, bool mesh);                        // per-(frame, slab) sums of the vertex error
// fold_m DEVICE [24][4] doubles, pairs DEVICE [n_pairs]; tab DEVICE [groups] (rc_motion_metrics' table); any output may be nullptr;
// mesh == false: no fold, no sweep, the mesh outputs are NaN
void rc_launch_aligned_metrics(const BodyConst* body, const float* vt, const float* w, int V, const double* fold_m, const AlignPair* pairs,
                               int n_pairs, const MotionGroup* tab, int groups, long long blocks, const float* pose_p, const float* pose_t,
                               long long n, unsigned what, bool mesh, float* scratch, double* partial, float* joint_err, float* mesh_err,
                               float* per_frame, float* xform, hipStream_t st);

// smplify optimiser (rc_smplify.hip): one evaluation = loss terms + analytic gradient of all T frames
struct SmplifyArgs {
    const float* aa;        // [T,72] axis-angle (root first)
    const float* tran;      // [T,3]
    const float* kp;        // [T,33,3] pixels + confidence (ignored landmarks count as 0)
    const float* ref3d;     // [T,33,3] landmarks of the initial prediction
    const float* imu_aa;    // [T,18] axis-angle of the measured IMU orientations
    const float* means;     // [8,69]
    const float* prec;      // [8,69,72] precision matrices, rows padded (rc_smplify_set_prior)
    const float* prec_sym;  // [8,69,72] P + P^T, rows padded
    const float* lognll;    // [8] log(nll_weights)
    float* mj;              // [T,33,3] out (fwd) / in (grad)
    float* proj;            // [T,33,2]
    float* frame_loss;      // [T] reprojection + prior + angle + 3D of frame t
    float* imu_loss;        // [T] 0.25 * |aa(imu) - aa(G[ji])|^2
    float* smooth_loss;     // [T] smoothness terms of the pair (t-1, t)
    int* argmin;            // [T] mixture component of the prior            } written by the prior kernel,
    float* prior_ll;        // [T] min_m 0.5 d^T P_m d - log(nll_w_m)        } read by the forward / gradient kernels
    float* prior_g;         // [T,69] (P_m + P_m^T) d of that mixture        }
    float* fk;              // [T,2,24,9] local and global rotations of the forward kernel's primal, read by the gradient kernel
    float* grad_aa;         // [T,72]  } one flat vector [T*72 | T*3], the optimiser's parameter order
    float* grad_tran;       // [T,3]   } (temporal_smplify.py:141: [body_pose, tran])
    float K[9];
    unsigned long long ign_mask;   // landmarks whose confidence counts as zero (bit v)
    int T;
};
void rc_launch_smplify(const SmplifyArgs& A, const BodyConst* body, hipStream_t s);
// vector kernels of the device-resident L-BFGS (rc_smplify.hip)
#define RC_LBFGS_MAX_PAIRS 100             // history of the device-resident L-BFGS = torch.optim.LBFGS's default history_size
struct VecComb { const float* v[2 * RC_LBFGS_MAX_PAIRS + 1]; float c[2 * RC_LBFGS_MAX_PAIRS + 1]; int n_vec; };   // 2.4 KB kernel argument
struct VecJob { const float* a; const float* b; int op; int pad_; };     // op 0: sum a b, 1: max |a|, 2: sum |a|
// the same for all rows of a lock-step round of the batched optimiser (descriptor tables in device memory, the row from blockIdx.y)
struct VecOp { const float* a; const float* b; const float* c; float* out; float* out2; float t; int kind; long long n; };   // kind 0 axpy, 1 pair
struct VecCombRow { VecComb c; float* out; long long n; };
struct VecJobN { const float* a; const float* b; int op; int pad_; long long n; };
void rc_launch_smplify_rows(const SmplifyArgs* rows_dev, int n_rows, int T_max, const BodyConst* body, hipStream_t s);
void rc_launch_smplify_totals(const SmplifyArgs* rows_dev, int n_rows, double* out_dev, hipStream_t s);   // total loss per table entry, the host's summation order
// set-up and wrap-up of a batch of rows (rc_smplify_run_batch) in one launch each: what rc_smplify_run does per row with
// rc_launch_residual / rc_launch_R2aa / rc_launch_body_fk / rc_launch_aa2R and two device-to-device copies
struct SmplifyRowIO {
    const float* pose;      // [T,24,3,3] initial local rotations
    const float* tran;      // [T,3]
    const float* kp;        // [T,33,3]
    const float* imu_ori;   // [T,6,3,3]
    float* x;               // [T*75] optimiser parameters [axis-angle | translation]
    float* imu_aa;          // [T,18]
    float* joint;           // [T,24,3]
    float* ref3d;           // [T,33,3]
    float* res0;            // [T,33] residual before
    float* res1;            // [T,33] residual after
    float* pose_out;        // [T,24,3,3]
    float* tran_out;        // [T,3]
    float K[9];
    int T;
    int live;               // wrap-up: 0 = the pre-check rejected the row (nothing to do)
};
void rc_launch_smplify_begin_rows(const SmplifyRowIO* rows_dev, int n_rows, int T_max, const BodyConst* body, float sigma,
                                  unsigned long long ign_mask, hipStream_t s);
void rc_launch_smplify_end_rows(const SmplifyRowIO* rows_dev, int n_rows, int T_max, const BodyConst* body, float sigma,
                                unsigned long long ign_mask, hipStream_t s);
void rc_launch_vec_ops(const VecOp* ops_dev, int n_ops, long long n_max, hipStream_t s);
void rc_launch_vec_comb_rows(const VecCombRow* rows_dev, int n_rows, long long n_max, hipStream_t s);
void rc_launch_vec_dots_rows(const VecJobN* jobs_dev, int n_jobs, int nb_max, double* partial, hipStream_t s);
void rc_launch_vec_axpy(const float* x, const float* d, float t, float* out, long long n, hipStream_t s);
void rc_launch_vec_pair(const float* g_new, const float* g_old, const float* d, float t, float* y, float* sv, long long n, hipStream_t s);
void rc_launch_vec_comb(const VecComb& c, float* out, long long n, hipStream_t s);
void rc_launch_vec_dots(const VecJob* jobs_dev, int n_jobs, long long n, double* partial, hipStream_t s);
// synthetic closure of rc_lbfgs_device_probe (rc_smplify.hip): reads aa = x, kp = a, ref3d = b, K[0] = 0.5 / T; fills grad_aa and the [3 T] terms
void rc_launch_syn_closure(const SmplifyArgs& A, hipStream_t s);
void rc_launch_syn_closure_rows(const SmplifyArgs* rows_dev, int n_rows, int T_max, hipStream_t s);

// ---- owners of the host code's HIP resources ----------------------------------------------------------------------------------------
// Move-only; resetting or destroying the owner releases the resource (return code ignored). Never give an owner static storage duration:
// its destructor would run after the HIP runtime has been torn down at exit. Kernel arguments take the raw pointer: .get().
template <auto Release> struct RcRelease { template <class P> void operator()(P p) const { (void)Release(p); } };
template <class T> using DevBuf = std::unique_ptr<T[], RcRelease<hipFree>>;        // hipMalloc
template <class T> using PinBuf = std::unique_ptr<T[], RcRelease<hipHostFree>>;    // hipHostMalloc
using HipStream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, RcRelease<hipStreamDestroy>>;
using HipEvent = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, RcRelease<hipEventDestroy>>;
using HipGraph = std::unique_ptr<std::remove_pointer_t<hipGraph_t>, RcRelease<hipGraphDestroy>>;
using HipGraphExec = std::unique_ptr<std::remove_pointer_t<hipGraphExec_t>, RcRelease<hipGraphExecDestroy>>;

// out-parameter of a create call, e.g. hipEventCreate(rc_out(ev)): the previous handle is released first, the new one is owned from the
// end of the statement
template <class Own> struct RcOut {
    Own& own;
    typename Own::pointer raw;
    ~RcOut() { own.reset(raw); }
    operator typename Own::pointer*() { return &raw; }
};
template <class Own> RcOut<Own> rc_out(Own& own) { own.reset(); return {own, nullptr}; }

// the previous buffer is released first; the contents are not kept
template <class T> hipError_t rc_alloc(DevBuf<T>& p, size_t n) {
    p.reset();
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, n * sizeof(T));
    p.reset(static_cast<T*>(q));
    return e;
}
template <class T> hipError_t rc_alloc(PinBuf<T>& p, size_t n, unsigned flags = hipHostMallocDefault) {
    p.reset();
    void* q = nullptr;
    const hipError_t e = hipHostMalloc(&q, n * sizeof(T), flags);
    p.reset(static_cast<T*>(q));
    return e;
}
inline hipError_t rc_alloc_all() { return hipSuccess; }
template <class Buf, class... Rest> hipError_t rc_alloc_all(Buf& p, size_t n, Rest&&... rest) {
    const hipError_t e = rc_alloc(p, n);
    return e != hipSuccess ? e : rc_alloc_all(rest...);
}
// Grow-only buffers that share one capacity (contents not kept): if cap < need, each buffer is allocated anew for the count that follows
// it, and cap becomes `want`. cap stays 0 until every allocation succeeded, so a failed growth is retried whole.
template <class Cap, class... BufsAndCounts> hipError_t rc_grow(Cap& cap, size_t need, size_t want, BufsAndCounts&&... bc) {
    if (need <= (size_t)cap) return hipSuccess;
    cap = 0;
    const hipError_t e = rc_alloc_all(bc...);
    if (e == hipSuccess) cap = (Cap)want;
    return e;
}
// A table the host builds per call and sends to the device on the caller's stream: the device table, a ring of `Ring` pinned copies, one
// event per copy (created with its first use; it says that the last upload from the copy, or whatever the site recorded it behind, is
// done) and the cursor. A call takes the next copy, so it waits for the call made `Ring` calls earlier and not for the one before it.
// Everything is grow-only, room for Slack * n entries where n are needed. The owner never synchronises a stream or the device: the
// device table may only grow behind the site's own synchronisation (kernels of earlier calls may still read the old one), which the
// site's contract in the header names. A call: stage -> fill -> [holds? -> the site synchronises -> grow] -> upload -> record.
#pragma GCC visibility push(hidden)
template <class T, int Ring, int Slack = 2> class StagedTable {
    static_assert(std::is_trivially_copyable<T>::value && Ring >= 1 && Slack >= 1, "plain entries, at least one pinned copy");
    DevBuf<T> dev_;
    size_t dev_n_ = 0;
    PinBuf<T> pin_[Ring];
    size_t pin_n_[Ring] = {};
    HipEvent ev_[Ring];
    int next_ = 0;
    int slot() const { return (next_ + Ring - 1) % Ring; }       // the copy the last stage() took
public:
    // the next pinned copy, free of its last upload and with room for n entries (the cursor moves before anything can fail)
    hipError_t stage(size_t n, T** host) {
        const int s = next_;
        next_ = (s + 1) % Ring;
        *host = nullptr;
        hipError_t e = ev_[s] ? hipEventSynchronize(ev_[s].get()) : hipEventCreateWithFlags(rc_out(ev_[s]), hipEventDisableTiming);
        if (e == hipSuccess) e = rc_grow(pin_n_[s], n, Slack * n, pin_[s], Slack * n);
        if (e == hipSuccess) *host = pin_[s].get();
        return e;
    }
    bool holds(size_t n) const { return n <= dev_n_; }
    hipError_t grow(size_t n) { return rc_grow(dev_n_, n, Slack * n, dev_, Slack * n); }
    hipError_t upload(size_t n, hipStream_t st) {
        return hipMemcpyAsync(dev_.get(), pin_[slot()].get(), n * sizeof(T), hipMemcpyHostToDevice, st);
    }
    hipError_t record(hipStream_t st) { return hipEventRecord(ev_[slot()].get(), st); }
    T* get() const { return dev_.get(); }
    size_t capacity() const { return dev_n_; }                    // entries of the device table
};
#pragma GCC visibility pop

// the live session of a context (rc_live_api.cpp; the type is complete there only)
struct LiveSession;
__attribute__((visibility("hidden"))) void rc_live_free(LiveSession* s);   // delete s
using LiveOwner = std::unique_ptr<LiveSession, RcRelease<rc_live_free>>;

// the sequence engine of a context (rc_sequence_api.cpp; the type is complete there only)
struct SeqEngine;
__attribute__((visibility("hidden"))) void rc_seq_free(SeqEngine* e);      // delete e
using SeqOwner = std::unique_ptr<SeqEngine, RcRelease<rc_seq_free>>;

// the gate-GEMM launcher of a context (rc_gemm_api.cpp; the type is complete there only)
struct GemmLauncher;
__attribute__((visibility("hidden"))) void rc_gemm_free(GemmLauncher* g);  // delete g
using GemmOwner = std::unique_ptr<GemmLauncher, RcRelease<rc_gemm_free>>;

// narrow view of the context for rc_smplify_api.cpp and rc_subnet_api.cpp (the struct itself lives in rc_ctx.h)
struct rc_ctx;
struct SmplifyState;
const BodyConst* rc_ctx_body(rc_ctx* ctx);                 // nullptr until rc_set_body
int rc_ctx_fail(rc_ctx* ctx, int code, const char* msg);   // records the message, returns code
#define HIP_TRY(ctx, expr)                                                                                                              \
    do {                                                                                                                                \
        const hipError_t e_ = (expr);                                                                                                   \
        if (e_ != hipSuccess) return rc_ctx_fail(ctx, RC_ERR_HIP, (std::string(#expr) + ": " + hipGetErrorString(e_)).c_str());       \
    } while (0)
void rc_smplify_free(SmplifyState* s);                     // delete s (the type is complete in rc_smplify_api.cpp only)
using SmplifyOwner = std::unique_ptr<SmplifyState, RcRelease<rc_smplify_free>>;
SmplifyOwner& rc_ctx_smplify(rc_ctx* ctx);
unsigned long long rc_ctx_ign_mask(rc_ctx* ctx);

// ---- sub-net forward over ragged sequences (rc_subnet.hip, rc_subnet_api.cpp; articulate/utils/torch/rnn.py:121-133) ----------------
// One tall GEMM: rows = frames of a time chunk (or the active prefix of one time step), workgroups of 64 * mr rows x 16 * nc columns,
// the weight k-blocks of a column tile staged once per workgroup in LDS and applied to all its rows. It forms the K quarters
// [c0, c1) of the packed weights (the per-wave chains of gemm_tile: quarter q = packed k [q Kp / 4, (q + 1) Kp / 4)) with the chains'
// instructions (rc_mma.h) and sums them in gemm_tile's order, so every output has the bits of the stepped launches.
enum { RC_SG_DENSE = 0, RC_SG_RELU = 1, RC_SG_HALF = 2, RC_SG_LSTM = 3,
       RC_SG_BPLAIN = 4, RC_SG_BSTEP = 5 };   // backward through time (rc_subnet_backward): the kernel's BWD instantiation
struct SubGemm {
    const float* A;          // rc_pk order, [rows, lda]; the chains read A column k - a_koff for packed k
    int lda, a_koff, M;
    const float* W;          // pack_weights (mode 0)
    const void* Ws;          // pack_weights_split (mode 1)
    int Kp, ncb;             // packed K (all four quarters), 16-column blocks of the packing
    int c0, c1;              // quarters formed here
    int N;                   // valid output columns
    int epi;                 // RC_SG_*
    const float* bias;       // packed column order (DENSE / RELU / LSTM)
    float* out;              // DENSE / RELU: rc_pk(row', col, ldo) if out_packed else row' * ldo + col, row' = out_map ? out_map[row] : row
    int ldo, out_packed;     // HALF: out[row * ldo + col] = q0 + q1 (the x half of a layer step, no bias)
    const int* out_map;
    // LSTM (a layer step over rows 0 .. M - 1 = the active prefix): gates = (pre[row * ldp + col] + (q2 + q3)) + bias
    const float* pre;
    int ldp, H;
    float* cst;              // [rows, H] in place
    float* hout;             // h(t): rc_pk(row, unit, H)
    float* hseq;             // ... and the chunk's sequence buffer rc_pk(hseq_row0 + row, unit, H)
    long long hseq_row0;
    // LSTM, recording (rc_subnet_forward_tape; null otherwise): the step's rows of the tape, in plan order
    float* tape_g;           // [rows, 4H] gate activations, packed column order (unit * 4 + i, f, g, o)
    float* tape_c;           // [rows, H] c(t)
    // BPLAIN: out[row' * ldo + col] = ((q0 + q1) + q2) + q3, row' = out_map ? out_map[row] : row (no bias)
    // BSTEP (one reverse step of a layer over the active prefix; A = dG(t + 1) in rc_pk order, weights = the transposed pack's W_hh
    // columns): dh = (row < n_next ? sum : dfin_h[row, u]) + dh_above, then the per-unit recurrences of rc_lstm_cell_backward on the
    // step's tape rows (tape_g, tape_c; c_prev) and the carried dc (cst, in place); dG(t) goes to hout (rc_pk, the next step's A),
    // hseq (the chunk's buffer) and dgates (the caller's rows, torch's column order g * H + u)
    int n_next;              // rows still running at step t + 1 (the others enter here with dfin_h and the dc the state was set to)
    const float* dfin_h;     // [rows, H]
    const float* dh_above;   // [*, H]: row dha_map ? dha_map[row] : row
    const int* dha_map;
    const float* c_prev;     // [rows, H]: c(t - 1) of the step's rows (the tape's previous step, or init_c by rank)
    float* dgates;           // [*, 4H] at row out_map[row]
};
void rc_launch_subnet_gemm(const SubGemm& G, int split, int tall, hipStream_t s);   // tall: 256-row tiles whatever M
void rc_launch_subnet_gemm_bwd(const SubGemm& G, int split, int tall, hipStream_t s);   // epi RC_SG_BPLAIN / RC_SG_BSTEP, the same tile dispatch
// dst[map[j] * cols + k] = src[rc_pk(j, k, ld)] for j < rows, k < cols (a chunk's sequence buffer -> the caller's rows)
void rc_launch_subnet_unpack(const float* src, int ld, const int* map, float* dst, int cols, int rows, hipStream_t s);
// backward state of ranks [0, nr) <-> sequences perm[r] (n: sequences in src / dst, [2, n, H]; a, b: per layer [rows, H], ls floats apart).
// in = 1: a, b (either may be null) from src_a, src_b (zeros where null); in = 0: dst_b (may be null) from b
void rc_launch_subnet_bstate(float* a, float* b, long long ls, const float* src_a, const float* src_b, float* dst_b, const int* perm,
                             int nr, int n, int H, int in, hipStream_t s);
// transposed operand of an LSTM layer from its fp32 packing Wl (Np = 4H, Kp = 2H): the same packing with Np = 2H, Kp = 4H of
// WT[n'][k'] = Wl's value at (column k', k = n'), as the fp32 pack WT and the three bf16 planes WTs
void rc_launch_subnet_transpose(const float* Wl, int H, float* WT, void* WTs, hipStream_t s);
// dst[rc_pk(j, k, ld)] = k < cols ? src[map[j] * cols + k] : 0 for j < rows, k < ld (user rows -> zero-padded A operand)
void rc_launch_subnet_pack(const float* src, int cols, const int* map, float* dst, int ld, int rows, hipStream_t s);
// state of sequence perm[r] <-> row r < nr (n: sequences in h, c). hp: per layer (hp + l * hl) two copies of h in rc_pk order, ps floats apart; cp: per layer
// (cp + l * cl) c [rows, H]; h, c: [2, n, H] in the caller's order. in = 1: copy 1 of hp and cp from h, c (zeros where null);
// in = 0: h, c (either may be null) from copy par[r] of hp and from cp
void rc_launch_subnet_state(float* hp, long long hl, long long ps, const int* par, float* cp, long long cl, float* h, float* c,
                            const int* perm, int nr, int n, int H, int in, hipStream_t s);
// in-place repack on the device (rc_update_subnet_weights): the index arithmetic and truncation split of pack_weights / pack_weights_split
void rc_launch_repack_dense(const float* Wsrc, int N, int K, int Np, int Kp, float* W, void* Ws, hipStream_t s);
void rc_launch_repack_lstm(const float* wi, const float* wh, const float* bi, const float* bh, int H, float* W, void* Ws, float* bl,
                           hipStream_t s);
// dropout of a trainable sub-net (rc_dropout.hip): kept iff Philox4x32-10(key = seed, counter = (row', k >> 2, site, call))[k & 3] >=
// round(p 2^32), row' = map ? map[j] : j (the frame's row in the caller's order); kept x / (1 - p), dropped +0. src == dst allowed;
// both 16-byte aligned, 0 < p < 1.
struct DropoutKey { float p; unsigned long long seed; unsigned call; };
// dst[j * cols + k] = drop(src[j * cols + k]) for j < rows, cols % 4 == 0
void rc_launch_dropout_rows(const float* src, float* dst, long long rows, int cols, const int* map, int site, const DropoutKey& k,
                            hipStream_t s);
// dst[rc_pk(j, k, ld)] = drop(src[rc_pk(j, k, ld)]) for j < rows (rows up to the 16-row padding are not touched), ld % 16 == 0
void rc_launch_dropout_pk(const float* src, float* dst, long long rows, int ld, const int* map, int site, const DropoutKey& k,
                          hipStream_t s);

// ---- weight gradients of a trainable sub-net (rc_wgrad.hip; rc_subnet_weight_grads in rc_subnet_api.cpp) --------------------------------
// C[M, N] = sum over frames f of A[f, m] * B'[f, n]: the contraction runs over the SLOW index of both row-major operands. B' is up to
// two column segments, each starting a 128-column tile of its own: rows as stored | rows masked at dropout site 1 while they are
// loaded | the rows of h shifted by one frame within each sequence (init_h, or zero, at a sequence's first frame). Frames are summed on
// two levels (256 frames in the MFMA accumulators, the blocks into a second set) and cut into `parts` ranges of whole blocks whose
// partial sums rc_launch_wgrad_reduce adds in index order. The column sums of A (the bias gradients) take the same two levels and
// parts in a kernel of their own, rc_launch_wgrad_colsum, on double accumulators.
#define RC_WG_TILE 128         // rows and columns of a workgroup's output tile (four waves, 64 x 64 each)
#define RC_WG_KB 32            // frames per staged LDS image
#define RC_WG_BLOCK 256        // frames per first-level sum
#define RC_WG_MAX_PARTS 16
enum { RC_WG_ROWS = 0, RC_WG_MASKED = 1, RC_WG_SHIFT = 2 };
struct WgradSeg {
    const float* src;        // [F, ld]
    const float* init;       // SHIFT: [sequences, ld] or null (zeros)
    float* out;              // [M, ldo]
    int ld, ncols, ldo, kind;
    int tile0;               // first column tile of the segment
    int vec;                 // src (and init) rows may be read as 16-byte pieces
};
struct WgradLaunch {
    const float* A;          // [F, lda], columns [0, M)
    int lda, M, a_vec;
    long long F;
    WgradSeg seg[2];
    int nseg, ntiles_n, ntiles_m;
    const int* first;        // [F]: the frame's sequence if it is the sequence's first frame, else -1
    int parts, blocks_per_part;
    float* partial;          // parts > 1: [parts][128 ntiles_m][128 ntiles_n]
    unsigned T;              // MASKED: kept iff bits >= T
    float scale;
    uint2 key;
    unsigned call;
};
void rc_launch_wgrad(const WgradLaunch& L, int split, hipStream_t s);           // parts == 1: writes the outputs itself
void rc_launch_wgrad_reduce(const WgradLaunch& L, hipStream_t s);               // parts > 1: outputs = partial sums added in index order
// out[m] (and out2[m], either may be null) = sum_f A[f, m], m < M: per part the 256-frame block sums added in frame order, the parts
// in index order (partial: [parts][M] doubles, used when parts > 1), rounded to fp32 once
void rc_launch_wgrad_colsum(const float* A, int lda, int M, long long F, int parts, int blocks_per_part, double* partial, float* out,
                            float* out2, hipStream_t s);

// ---- the optimiser step of one sub-net (rc_optim.hip; rc_subnet_optim_step in rc_api.cpp) -----------------------------------------------
#define RC_OPTIM_CHUNK 16384   // gradient elements per workgroup (and per partial sum) of the norm
#define RC_OPTIM_MAXT 18       // tensors of a sub-net at most (rnn2)
struct OptimNorm {             // the gradients in the caller's order; tensor t owns workgroups [block0[t], block0[t + 1]) -- none when skipped
    const float* g[RC_OPTIM_MAXT];
    long long n[RC_OPTIM_MAXT];
    int block0[RC_OPTIM_MAXT + 1];
    int count;
};
struct OptimTensor { float* p; const float* g; float* m; float* v; };   // parameter, gradient (null: the tensor is skipped), first and second moment
struct OptimScalars { float step_size, bc2_sqrt, beta1, one_m_beta1, beta2, one_m_beta2, eps, weight_decay; };   // step_size = lr / bc1
// partial [blocks] sums of squares in double, then out2 = {total norm, clip coefficient} (max_norm <= 0: coefficient 1)
void rc_launch_optim_norm(const OptimNorm& A, int blocks, double* partial, float max_norm, float* out2, hipStream_t s);
// clip (coefficient read from out2[1]), Adam in place and rc_launch_repack_lstm / rc_launch_repack_dense's stores in one pass
void rc_launch_optim_lstm(const OptimTensor& wi, const OptimTensor& wh, const OptimTensor& bi, const OptimTensor& bh, int H, float* W, void* Ws,
                          float* bl, const OptimScalars& a, const float* out2, hipStream_t s);
void rc_launch_optim_dense(const OptimTensor& Wt, const OptimTensor& bt, int N, int K, int Np, int Kp, float* W, void* Ws, float* Wrm, float* bp,
                           const OptimScalars& a, const float* out2, hipStream_t s);

// ---- the training objectives of the sub-nets (rc_loss.hip; rc_subnet_loss in rc_api.cpp) ---------------------------------------------------
// (the kinds: rc_loss_kind of the header, which rc_loss.hip and rc_api.cpp include)
#define RC_LOSS_VEC 4                // elements a thread moves at once (mse, bce_logits): one 16-byte piece
#define RC_LOSS_CHUNK 4096            // elements per unit of mse and bce_logits: four pieces per thread of a workgroup
#define RC_LOSS_WINDOW_FRAMES 240     // frames per unit of window_mse, counted from the end of the batch: four blocks of 60
#define RC_LOSS_POSE_FRAMES 16        // frames per unit of pose_fk: four per wave
#define RC_LOSS_MAX_PARTIALS 1024     // workgroups (and partial sums) of a call at most: beyond it a workgroup takes several units
// value = the loss of x, y [F, W] (one device float), dx (may be null) its gradient; partial: RC_LOSS_MAX_PARTIALS doubles
void rc_launch_subnet_loss(int kind, const BodyConst* body, const float* x, const float* y, long long F, int W, const float* aux,
                           double* partial, float* value, float* dx, hipStream_t s);
// ---- the validation metrics of the sub-nets, per group of a concatenated batch (rc_loss.hip; rc_subnet_eval in rc_api.cpp) -----------------
#define RC_EVAL_POINTS 1024           // 3-D points per unit of position_error: four per thread of a workgroup
#define RC_EVAL_MAX_GROUPS 65536      // groups of a call at most (at most RC_LOSS_MAX_PARTIALS workgroups each: the grid stays below 2^31)
// One group: frames [frame0, frame0 + frames) of x and y; its workgroups are [blk0, blk0 + nblk) of the launch, nblk = what rc_subnet_loss
// launches for such a slice; c: the double reciprocals rc_launch_subnet_loss hands its kernels for such a slice (element kinds and
// position_error: 1 / count | window_mse: 1 / (3 F), 1 / (3 (F / 6)), 1 / (3 (F / 20)), 1 / (3 (F / 60)) | pose_fk: 1 / (144 F), 100 / (72 F))
struct EvalGroup { long long frame0, frames; int blk0, nblk; double c[4]; };
void rc_eval_group(int kind, int W, EvalGroup* g);         // frames set by the caller -> nblk and c, by the code rc_launch_subnet_loss uses
// values[g] = the value of group g; tab DEVICE [groups]; blocks = sum of nblk; partial: `blocks` doubles. Two launches whatever `groups` is.
void rc_launch_subnet_eval(int kind, const BodyConst* body, const EvalGroup* tab, int groups, long long blocks, const float* x, const float* y,
                           int W, const float* aux, double* partial, float* values, hipStream_t s);

// ---- the training batches of one sub-net (rc_augment.hip; rc_subnet_batch in rc_subnet_api.cpp) ------------------------------------------
// tab (device): [n] first corpus frame of every sample | [n + 1] first output frame of every sample, then the total F. Draws: Philox4x32-10
// with key = seed and counter = (sample, frame within the sample, site | index << 8, call), sites 2 .. 6 (rc_augment.hip).
struct BatchKey { unsigned long long seed; unsigned call; };
struct BatchCamera { float yaw_lo, yaw_hi, pitch_lo, pitch_hi, roll_lo, roll_hi; };   // degrees
// x_out[f] = data[row of f], columns [c0, W) + sigma * normal (c0 == W: a copy); l_out[f] = label[row of f]. Any alignment.
// ext (device, or nullptr: rc_subnet_batch): the launch is one kind's share of a mixed batch (rc_subnet_batch_parts) -- [n] the sample's
// position in the whole batch (the Philox `sample` word) | [n] its first output frame in the whole batch | [n] its part's data | [n] its
// part's label (device addresses); tab's output frames then only enumerate the launch's own frames.
void rc_launch_batch_plain(const float* data, const float* label, const long long* tab, int n, long long F, int W, int Wl, int c0,
                           float sigma, const BatchKey& k, float* x_out, float* l_out, hipStream_t s, const long long* ext = nullptr);
// the AMASS sample of rnn4 (rnn4 != 0: x [F, 171], label [F, 69]) or rnn6 (x [F, 240], label [F, 3]) from data [., 171], label [., 72] and
// pool [pool_rows, 33]; cam: [n, 12] scratch (Rcw | t per sample), written by the first of the two launches
void rc_launch_batch_world(int rnn4, const float* data, const float* label, const long long* tab, int n, long long F,
                           const BatchCamera& range, float* cam, const float* pool, int pool_rows, float sigma, const BatchKey& k,
                           float* x_out, float* l_out, hipStream_t s, const long long* ext = nullptr);

// ---- the training corpus of one sub-net (rc_corpus.hip; rc_subnet_corpus in rc_subnet_api.cpp) -------------------------------------------
// tab (device): [n] first field frame of every sample's sequence | [n] first keypoint frame of every sample | [n + 1] first output row of
// every sample, then the total R. cams (device, camera mode): per sample K^-1 [9] | rows 0 .. 2 of T_cw [12] | 1.0 for an occlusion sample.
struct CorpusArgs {
    const float *pose, *acc, *ori, *joint, *tran, *mp, *kp;   // the fields, concatenated over the sequences (kp: over the samples)
    const long long* tab;
    const float* cams;
    const BodyConst* body;                                    // rnn7: the parent table
    int n, net, amass, W, Wl;                                 // samples, kNets index, the AMASS spelling, row widths
    long long R;
    float sx, sy;                                             // image size: keypoints are stored divided by it
    float *x, *y;
};
void rc_launch_subnet_corpus(int mode, const CorpusArgs& a, hipStream_t s);   // mode 0: root frame, 1: camera frame, 2: world
// K^-1, R_cw and gravity of one camera by rc_camera_inputs_rows' routine (rc_api.cpp); false, nothing written: unusable
bool rc_camera_constants(const float* K, const float* Tcw, CamConst* cam, float* g_out);

// narrow view of the context for rc_subnet_api.cpp
struct SubnetState;
struct SubnetDense { const float* W; const void* Ws; const float* b; int K, N, Kp, Np; };
struct SubnetNet { SubnetDense lin1, lin2; const float* Wl[2]; const void* Wls[2]; const float* bl[2]; int in, H, out; };
int rc_ctx_subnet_net(rc_ctx* ctx, int net, SubnetNet* out);     // net: kNets index (rnn2 .. rnn8); RC_ERR_STATE before weights
int rc_ctx_init_net(rc_ctx* ctx, SubnetDense out[3]);
int rc_ctx_net_index(const char* name);
int rc_ctx_gemm_split(rc_ctx* ctx);                        // 1: the context's products are not fp32 (gemm mode 1 or 2)
int rc_ctx_gemm_mode(rc_ctx* ctx);                         // rc_get_gemm_mode
int rc_ctx_flush_pending(rc_ctx* ctx, hipStream_t st);     // every pending updater step runs now, on st (rc_get_state, rc_set_state)
int rc_ctx_mark_eager(rc_ctx* ctx, hipStream_t st);        // mark_eager (rc_ctx.h): eager work was enqueued on st
long long rc_ctx_weights_epoch(rc_ctx* ctx);               // counts rc_finalize_weights: what was derived from the packed weights is stale
void rc_subnet_free(SubnetState* s);                       // delete s
using SubnetOwner = std::unique_ptr<SubnetState, RcRelease<rc_subnet_free>>;
SubnetOwner& rc_ctx_subnet(rc_ctx* ctx);
// the transposed packs of net ni that exist are rebuilt from the layers' fp32 packings Wl on stream s (rc_update_subnet_weights)
void rc_subnet_retranspose(SubnetState* S, int ni, const float* const Wl[2], int H, long long epoch, hipStream_t s);
