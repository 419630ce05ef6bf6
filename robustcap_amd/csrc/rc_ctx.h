// The context behind the C ABI, for the two files that work on all of it: rc_api.cpp and rc_live_api.cpp. (rc_smplify_api.cpp and
// rc_subnet_api.cpp see it through the rc_ctx_* accessors of rc_internal.h.)
#pragma once
#include "../../include/robustcap_hip.h"
#include "rc_internal.h"

#include <map>
#include <string>
#include <utility>
#include <vector>

struct NetSpec { const char* name; int in, H, out; };
const NetSpec kNets[6] = {{"rnn2", 72, 512, 69},  {"rnn3", 141, 512, 3},   {"rnn4", 171, 1280, 69},
                          {"rnn6", 240, 1024, 3}, {"rnn7", 141, 512, 144}, {"rnn8", 141, 512, 2}};
enum { N2 = 0, N3 = 1, N4 = 2, N6 = 3, N7 = 4, N8 = 5 };

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

struct Dense {       // packed dense layer
    float* W = nullptr; float* b = nullptr;
    void* Ws = nullptr;                  // split-bf16 planes of W
    float* Wrm = nullptr;                // narrow layers (linear2): the matrix as loaded, row-major [N][K] (rc_live.hip)
    int K = 0, N = 0, Kp = 0, Np = 0;
    int mr = 2, nc = 4;                  // tile shape: 16*mr rows x 16*nc columns
};
struct NetDev {
    Dense lin1, lin2;
    float* Wl[2] = {nullptr, nullptr};   // LSTM layers, K' = 2H, N' = 4H (tile-interleaved gates)
    void* Wls[2] = {nullptr, nullptr};   // their split-bf16 planes
    float* bl[2] = {nullptr, nullptr};
    float* h = nullptr;                  // [layer][copy of RC_HBUF][B][H]
    float* c = nullptr;                  // [layer][B][H]
    int* steps = nullptr;                // [B]
    float* x1 = nullptr;                 // relu(linear1) scratch [B][H]
    float* part = nullptr;               // lean live frame: per-tile partial sums of linear2 [H / 4][RC_LIVE_MAXB][outp]
    int in = 0, H = 0, out = 0;
    int nc = 4;                          // 16-column blocks per LSTM tile (4*nc hidden units x 4 gates)
    int mr = 2;                          // 16-row blocks per LSTM tile
};

struct rc_ctx {
    int B = 0;
    int Bp = 0;                          // B rounded up to the 32-row tile (row count of rc_pk buffers)
    int dev = 0;
    rc_params prm{};
    NetDev net[6];
    Dense init[3];
    float *hid1 = nullptr, *hid2 = nullptr, *xtmp = nullptr;
    FrameBuffers fb{};
    BodyConst* body = nullptr;
    float *mesh_vt = nullptr, *mesh_w = nullptr;      // full mesh (metrics only): v_template [V,3], weights [V,24]
    int mesh_V = 0;
    float* mesh_kM = nullptr;                         // keypoint regressor folded with the skinning data [n_used][24][4] (metrics only)
    int mesh_nk = 0;
    std::vector<float> mesh_vt_h, mesh_w_h, mesh_Jr_h; // host copies: the fold is recomputed when mesh, regressor or root change
    float jroot_h[3] = {0.f, 0.f, 0.f};
    bool fold_dirty = false;
    DevBuf<float> sweep_scratch;                      // per-frame transforms + slab partial sums of the mesh sweeps (grow-only)
    size_t sweep_scratch_cap = 0;
    unsigned long long ign_mask = RC_IGN_DEFAULT;     // smplify: landmarks with zeroed confidence
    bool have_body = false, have_weights = false;
    std::map<std::string, std::vector<float>> staged;    // host copy of the tensors loaded since the last rc_finalize_weights
                                                         // (released there: a context does not hold 254 MB of host memory)
    std::vector<DevBuf<char>> allocs;
    std::vector<std::pair<void*, size_t>> alloc_bytes;   // (pointer, bytes) of every dev_alloc that is not a weight: state + scratch
    std::vector<DevBuf<char>> weight_allocs;   // packed weights of the current rc_finalize_weights (freed by the next one)
    bool alloc_weights = false;          // dev_alloc books into weight_allocs
    std::string err;
    LiveOwner live;                      // the live session: stream, captures, packet chain, host mirror, knobs and counters (rc_live_api.cpp)
    // timing of the gate GEMM launches
    bool timing = false;
    int timing_mode = 1;                 // 1: every gate-GEMM launch, 2: only the wide-tile kernels, 3: only the shared-weight kernel (rc_gemm_lds_kernel)
    std::vector<std::pair<HipEvent, HipEvent>> ev_pool;
    size_t ev_used = 0;
    double timed_ms = 0.0;
    double timed_busy_ms = 0.0;          // time with at least one timed launch running (launches on two streams overlap)
    long long timed_launches = 0;
    // sequence mode of rc_sequence: launch planner + per-row-cursor wavefront engine (run_wave2_segment)
    bool gemm_split = false;             // products of every GEMM as split-bf16 partial products (rc_set_gemm_mode)
    bool live_launch = false;            // set while a live frame is captured / launched (GemmLaunch.live)
    unsigned live_nt_mask = 63u;         // sub-nets (bit = kNets index) whose weights a live frame streams with non-temporal loads
    int seq_mode = 1;                    // 0 = always frame-stepped, 1 = plan per call (cost estimate), 2 = wavefront whenever long enough
    int seq_min_frames = 8;              // calls shorter than this are neither planned nor skewed (no pre-pass, no synchronisation)
    float* x1_alt[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // second relu(linear1) buffer per net
    int tile6[2] = {0, 0}, tile378[2] = {0, 0}, tile2[2] = {0, 0}, tile4[2] = {0, 0};   // LSTM tile shapes of full-batch stages (0 = pick_tile)
    bool ring2_failed = false;           // ensure_wave2_buffers failed once: not retried
    // streams of a tick beside the caller's (stream_tick; caller's stream: plain both wide launches | split {rnn6, rnn4, init_net} | tri rnn4)
    HipStream aux_stream;                // the second stream, every engine: prep, linear2, fuse, tail; tri also {linear1, init_net} at the head of its tick
    HipStream wide2_stream;              // plain: unused | split: {H = 512 nets, linear1} | tri: rnn6
    HipEvent ev_main[8], ev_aux[8], ev_wide2[4];   // [tick & 3]: the last wide launch of the caller's stream | the end of aux_stream's tick | wide2_stream's
                                                   // launch is done (ev_main[6], [7]: the engine's streams join the caller's)
    HipStream wide3_stream;              // tri only: the H = 512 nets
    HipEvent ev_head[4], ev_wide3[4];    // tri only: {linear1, init_net} at the head of aux_stream's tick | wide3_stream's launch is done
    float* x1_alt2[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // third relu(linear1) buffer per net (linear1 runs up to a tick ahead of its readers)
    DevBuf<signed char> scan_codes_d;    // [cap] regime code per (frame, row)
    PinBuf<signed char> scan_codes_h;    // pinned
    PinBuf<int> scan_state_h;            // pinned: first_reach[B] then pend[B] (as ints)
    size_t scan_cap = 0;
    long long stat_wave_frames = 0, stat_stepped_frames = 0, stat_ticks = 0;
    long long stat_row_frames = 0;       // row-frames computed by sequence calls (rc_get_sequence_row_frames)
    // rc_sequence_rows: the call's per-row lengths, device + pinned (grow-only, released with the context). The pinned copy has two halves
    // that calls take in turn, each with an event that says its upload has left it: a call only ever waits for the upload of the call
    // BEFORE the previous one, which has long run.
    DevBuf<int> row_len_d;
    PinBuf<int> row_len_h;               // [2][row_len_cap]
    size_t row_len_cap = 0;
    HipEvent row_len_ev[2];
    unsigned row_len_turn = 0;
    // per-row-cursor wavefront engine (run_wave2_segment)
    bool ring2_ready = false;
    FrameBuffers ring2[16];              // ring slots: inter-stage buffers, updater inputs, frame index and step numbers per row
    std::vector<GemmProblem> wave2_prob; // [16 slots][W2_PROB]
    bool wave2_valid = false;
    DevBuf<int> frame_at_d;              // [cap] host plan: frame every row starts at every tick
    PinBuf<int> frame_at_h;              // pinned
    size_t frame_at_cap = 0;
    double cost_tick_us = 1.0, cost_tick_small_us = 13.0, cost_frame_us = 285.0, cost_tr_us = 55.0;   // engine choice (plan_wave): scale of the
                                                         // per-layer tick estimate, hand-over per tick, frame-stepped frame, its transition launches
    SmplifyOwner smplify;                // optimiser work space (rc_smplify_api.cpp)
    SubnetOwner subnet;                  // scratch of rc_subnet_forward (rc_subnet_api.cpp)
    int trace_next = 0;                  // tile-trace slot counter (tools/tile_trace.py)
    long long stat_wide_launches = 0;    // launches of the wide-tile kernels (rc_get_launch_stats)
    // shared-weight gate GEMM (rc_gemm_lds.hip): LSTM layer steps of >= lds_min_rows rows in split-product mode
    // Two thresholds (round 6, second session; tools/ab_batch.py): a CONTEXT takes the shared-weight kernel and the three-stream tick from
    // lds_min_batch rows (batch 64 loses a sixth with them: 688k -> 576k mixed), and inside such a context a PROBLEM runs on it from
    // lds_min_rows rows (the rnn4 / rnn6 problems of a mixed batch hold only the rows that see the camera). One threshold of 160 for both
    // (first session) left batch 96-128 on the 64-row tiles: batch 128 mixed 858k -> 933k, all-visible 1,073k -> 1,173k; 96: 691k -> 752k.
    int lds_min_rows = 64;               // RC_LDS_MIN_ROWS (0 = never); default: half the batch, within 64 .. 160 (batch 256: 128 = 160 within the noise, 64 costs 0.7 %)
    int lds_min_batch = 65;              // RC_LDS_MIN_BATCH: batch 72 / 80 / 88 mixed 528 / 587 / 653k on 64-row tiles (two row tiles, the second mostly padding) -> 585 / 654 / 691k;
                                         // 64 rows and fewer keep the one-reader 64-row launches (688k against 576k)
    int lds_ksplit[3] = {1, 2, 2};       // RC_LDS_KSPLIT_512 / _1024 / _1280: workgroups per tile (1: both K halves in one workgroup; the H = 512
                                         // nets' items are short -- 2 x 16 k-blocks -- and a hand-over per tile costs more than it levels: +1 %)
    DevBuf<float> lds_slab;              // [kLdsRegions][lds_region_tiles][RC_LDS_SLAB_FLOATS]: half sums in flight, one region per launch
    DevBuf<int> lds_tickets;             // [kLdsRegions][lds_region_tiles]
    size_t lds_region_tiles = 0;
    unsigned lds_rot = 0;
    // resident layer-step kernel of the wavefront engine (run_resident_segment)
    DevBuf<ResidentTick> res_ticks_d;        // [res_cap]
    PinBuf<ResidentTick> res_ticks_h;        // pinned
    DevBuf<int> res_ints_d;                  // item_base [res_cap + 1] | done [res_cap][RC_RES_MAXP] | tick_done [res_cap] | head, flag_l1, flag_tail, abort
    PinBuf<int> res_base_h;                  // pinned: item_base
    PinBuf<int> res_abort_h;                 // pinned: the abort word of the last segment (allocated with the first resident segment)
    size_t res_cap = 0;
    long long stat_resident_segments = 0, stat_resident_aborts = 0;
    bool resident_on = false;                // rc_set_resident / RC_SEQ_RESIDENT
    int resident_wgs = 224;                  // workgroups of the resident kernel (RC_SEQ_RESIDENT_WGS; the CUs it leaves run the second stream)
    long long stat_lds_launches = 0;
    long long stat_w32_launches = 0;         // of the wide launches: those on rc_gemm_split48_w32_kernel (contexts of 33-64 rows)
};

#pragma GCC visibility push(hidden)
// rc_api.cpp
int fail(rc_ctx* ctx, int code, const std::string& msg);      // records the message (ctx == nullptr: for rc_last_error(nullptr)), returns code
int tune_env(const char* name, int dflt);
int check_ready(rc_ctx* ctx);
rc_params_dev dev_params(const rc_params& p);
int step_impl(rc_ctx* ctx, const FrameIO& io, uint32_t flags, hipStream_t st, bool with_tr = true, bool skip_prep = false,
              const FrameIO* next_io = nullptr, int n_live = -1);
// rc_live_api.cpp
void live_create(rc_ctx* ctx);                                // rc_create: the RC_LIVE_* knobs are read here, once per context
void live_forget_last_frame(rc_ctx* ctx, bool rows_reset = false);   // an eager entry is about to move the state: the host mirror no longer knows
                                                              // the last frame (rows_reset: and any row may trigger init_net again)
int live_discard_ahead(rc_ctx* ctx);                          // what the session computed or queued ahead of the next frame no longer holds
int mark_eager(rc_ctx* ctx, hipStream_t st);                  // live_discard_ahead + the next live frame waits for the work just enqueued on st
#pragma GCC visibility pop
